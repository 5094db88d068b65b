"""Multiple importance sampling of lights on the device against its restatement.

tests/golden/mis_restate.py states the estimator in numpy f32; tests/golden/make_mis_golden.py ran it into
mis_golden_<scene>.npz.  With option "mis" on the device has to give the same bits in film, weight, final
sampler state and (counting build) closest-hit and shadow ray counts, whatever options, builder, session split
or context split is used; with it off, or where no vertex is paired, today's bits.
"""
import subprocess
import sys

import numpy as np
import pytest

from akari_amd import capi, envmap, progressive, render, scene
from conftest import CORNELL_MESH, GOLDEN, ROOT
from test_denoise_host import relmse
from test_gpu_path_kat import probe_frame
from test_path_kat_host import M, check, compare_with_golden, golden

sys.path.insert(0, str(GOLDEN))
import make_env_golden as ME  # noqa: E402
import make_mis_golden as MM  # noqa: E402
import mis_restate as S  # noqa: E402
import ref_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = list(MM.CONFIGS)


def mis_golden(name):
    return np.load(GOLDEN / f"mis_golden_{name}.npz")


def upload(ctx, name, key, sp=0.5, **build_kw):
    cs = scene.compile_scene(MM.build_scene(name, key, sp))
    scene.upload_scene(ctx, cs, **build_kw)
    return cs


def render_and_compare(factory, name, what, counting=(0,), exact_cull=False, options=None, **build_kw):
    """Every configuration of the scene with the switch on, each in a context of its own (a context holds one
    scene); `counting`: the values of count_tests to render with."""
    g = mis_golden(name)
    for key, env_on, sp, depth, clamp in MM.CONFIGS[name]:
        with factory(0) as ctx:
            for k, v in (options or {}).items():
                ctx.set_option(k, v)
            ctx.set_option("mis", 1)
            ctx.set_option("pixel_probe", 1)
            upload(ctx, name, key, sp, **build_kw)
            mask = g[key + "_mask"]
            H, W = mask.shape
            for c in counting:
                ctx.set_option("count_tests", c)
                rad, w = ctx.render(MM.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp, exact_cull=exact_cull)
                rays = compare_with_golden(g, key, mask, rad, w, probe_frame(ctx, W, H), f"{name} {key} {what} count {c}")
                assert ctx.render_form()["form"] == "wavefront", ctx.render_form()
                if c:
                    assert rays, f"{what}: the counting build recorded no ray counts"


@pytest.mark.parametrize("name", SCENES)
def test_scenes_equal_golden_default_options(hip_ctx_factory, name):
    render_and_compare(hip_ctx_factory, name, "default options", counting=(0, 1))


@pytest.mark.parametrize("name", SCENES)
def test_scenes_equal_golden_path_forced_and_exact_cull(hip_ctx_factory, name):
    """`path` 1 asks for the persistent kernel; with the switch on the wavefront form runs and says so."""
    render_and_compare(hip_ctx_factory, name, "path 1 forced", options={"path": 1, "path_defer": 0, "path_spec": 0})
    render_and_compare(hip_ctx_factory, name, "exact_cull", exact_cull=True)


@pytest.mark.parametrize("builder", ["sbvh", "lbvh"])
@pytest.mark.parametrize("name", SCENES)
def test_builders_equal_golden(hip_ctx_factory, name, builder):
    kw = {"sbvh": dict(builder=capi.BUILDER_SBVH), "lbvh": dict(builder=capi.BUILDER_LBVH)}[builder]
    render_and_compare(hip_ctx_factory, name, builder, **kw)


def test_unpaired_depths_and_switch_off_give_todays_bits(hip_ctx_factory):
    """At max_depth 0 and 1 no vertex is paired, so the switch changes no bit of the existing goldens; it is
    rendered after a deep render in the same context, whose terminal terms must not leak into it (E is zeroed
    per pass).  And a fresh session with the switch off again is today's render, persistent form included."""
    ge, gp = np.load(GOLDEN / "env_golden_cornell.npz"), golden("cornell")
    H, W = ge["mask"].shape
    tiles = [(0, 0, W, H)]
    with hip_ctx_factory(0) as ctx:
        ctx.set_option("pixel_probe", 1)
        ctx.set_option("mis", 1)
        upload(ctx, "cornell", "p50d5")
        for key, sp, depth, clamp in ME.CONFIGS["cornell"]:
            if depth > 1 or sp != 0.5:
                continue
            ctx.render(MM.SPP, 5, tiles, W, H)          # terminal terms in most slots, both pass parities
            rad, w = ctx.render(ME.SPP, depth, tiles, W, H, ray_clamp=clamp)
            compare_with_golden(ge, key, ge["mask"], rad, w, probe_frame(ctx, W, H), f"mis on, environment, {key}")
        ctx.set_option("mis", 0)
        key, sp, depth, clamp = ME.CONFIGS["cornell"][2]
        rad, w = ctx.render(ME.SPP, depth, tiles, W, H, ray_clamp=clamp)
        compare_with_golden(ge, key, ge["mask"], rad, w, probe_frame(ctx, W, H), f"mis off after on, {key}")
    with hip_ctx_factory(0) as ctx:
        ctx.set_option("pixel_probe", 1)
        upload(ctx, "cornell", "noenv_d5")
        for k, v in {"path": 1, "path_defer": 0, "path_spec": 0}.items():
            ctx.set_option(k, v)
        ctx.set_option("mis", 1)
        for depth in (0, 1):
            rad, w = ctx.render(M.SPP, depth, tiles, W, H)
            assert ctx.render_form()["form"] == "wavefront"
            compare_with_golden(gp, M.cfg_key(depth, 0.0), gp["mask"], rad, w, probe_frame(ctx, W, H), f"mis on, d{depth}")
        ctx.set_option("mis", 0)
        rad, w = ctx.render(M.SPP, 5, tiles, W, H)
        assert ctx.render_form()["form"] == "k_path", ctx.render_form()
        compare_with_golden(gp, "d5", gp["mask"], rad, w, probe_frame(ctx, W, H), "mis off after on, k_path")


def test_continue_keeps_the_sessions_value_and_film_variance_changes_no_bit(hip_ctx_factory):
    name, (key, _, sp, depth, clamp) = "cornell", MM.CONFIGS["cornell"][2]
    g = mis_golden(name)
    H, W = g[key + "_mask"].shape
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, key, sp)
        ctx.set_option("pixel_probe", 1)
        ctx.set_option("mis", 1)
        ctx.render(2, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
        ctx.set_option("mis", 0)                        # read when the session starts: the continue is still MIS
        rad, w = ctx.render_continue(2, W, H)
        assert ctx.render_form()["form"] == "wavefront"
        check(rad, g[key + "_radiance"], "2 + 2 spp by render_continue: radiance")
        check(w, g[key + "_weight"], "2 + 2 spp by render_continue: weight")
        assert np.array_equal(probe_frame(ctx, W, H)["seed"], g[key + "_seed"]), "2 + 2 spp: final sampler states"
        ctx.set_option("mis", 1)
        ctx.set_option("film_variance", 1)
        rad, w = ctx.render(MM.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
        compare_with_golden(g, key, g[key + "_mask"], rad, w, probe_frame(ctx, W, H), "film_variance on")
        assert ctx.render_variance(W, H).shape == (H, W, 4)
        for bad in (2, -1):
            with pytest.raises(capi.AkrError, match="mis must be in"):
                ctx.set_option("mis", bad)


def test_two_context_split_equals_single(hip_ctx_factory):
    name, (key, _, sp, depth, clamp) = "sky", MM.CONFIGS["sky"][0]
    g = mis_golden(name)
    H, W = g[key + "_mask"].shape
    tiles = [(x, y, x + 8, y + 8) for y in range(0, H, 8) for x in range(0, W, 8)]
    with hip_ctx_factory(0) as a, hip_ctx_factory(0) as b:
        upload(a, name, key, sp)
        upload(b, name, key, sp)
        rad, w = capi.render_node([a, b], MM.SPP, depth, tiles, W, H, ray_clamp=clamp, mis=True)
        check(rad, g[key + "_radiance"], "two-context render_node radiance")
        check(w, g[key + "_weight"], "two-context render_node weight")


_PREFIX = {}


def sky_prefixes(cap):
    """The restatement's `sky` d3 film sums and sampler states after 1 .. cap samples of every pixel, run once:
    a slot's samples are one chain, so a slot that holds c samples equals entry c whatever its neighbours hold."""
    if cap not in _PREFIX:
        key, _, sp, depth, clamp = MM.CONFIGS["sky"][0]
        sc = R.RefScene(MM.build_scene("sky", key, sp))
        env = ME.restated_env("sky", sp)
        W, H = sc.camera.res
        film = np.zeros((cap + 1, H, W, 3), np.float32)
        seed = np.zeros((cap + 1, H, W), np.uint32)
        for y in range(H):
            for x in range(W):
                sampler, tr, rad = R.LCG(x + y * W), R.Tracer(sc), (R.F(0.0),) * 3
                seed[0, y, x] = sampler.seed
                for c in range(1, cap + 1):
                    L = S.path_sample(sc, sampler, x, y, depth, None, tr, None, None, env, True)
                    rad = R.add(rad, L)
                    film[c, y, x], seed[c, y, x] = rad, sampler.seed
        film.setflags(write=False)
        seed.setflags(write=False)
        _PREFIX[cap] = (film, seed, depth)
    return _PREFIX[cap]


def check_per_slot(ctx, film, seed, w, rad, what):
    """Every slot against the restatement at the slot's own count (whole-frame tile: slot = y * W + x)."""
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
        upload(ctx, "sky", "d3")
        ctx.set_option("mis", 1)
        ctx.render(2, depth, tiles, W, H)
        mask = (np.arange(W * H) % 3 == 0).astype(np.uint8)
        rad, w = ctx.render_continue_masked(2, mask, W, H)
        assert ctx.render_form()["form"] == "wavefront"
        count = check_per_slot(ctx, film, seed, w, rad, "masked continue")
        assert np.array_equal(count.reshape(-1), np.where(mask != 0, 4, 2))
        rad, w = ctx.render_continue(1, W, H)
        check_per_slot(ctx, film, seed, w, rad, "uniform continue of a masked session")
        seen = []
        rad, w, info = progressive.render_adaptive(ctx, cap, depth, tiles, W, H, 0.05, min_spp=2, pass_spp=2,
                                                   on_pass=lambda info, rad, w: seen.append(info["spp_max"]))
        count = check_per_slot(ctx, film, seed, w, rad, "stepwise adaptive")
        print(f"stepwise adaptive: passes {seen}, counts {np.unique(count, return_counts=True)}")
        assert info["samples"] == count.sum() and count.min() >= 2 and count.max() <= cap


# ----------------------------------------------------------------------------- quality on the device
def glossy_floor_scene(resolution):
    """make_env_golden's ground quad and box with a Glossy floor of roughness 0.1 and an all-Diffuse box,
    under procedural_sky(64): the BSDF lobe of the floor is far narrower than the sky is wide."""
    sc = ME.sky_scene(resolution)
    ct = scene.ConstantTexture
    mats = sc.shapes[0].materials
    mats[0] = scene.GlossyMaterial(ct([0.8, 0.8, 0.8]), ct([0.1, 0.1, 0.1]))
    mats[2] = scene.DiffuseMaterial(ct([0.7, 0.6, 0.5]))
    sc.environment = scene.EnvironmentLight(envmap.procedural_sky(64), layout="octahedral")
    return sc


def test_quality_glossy_floor_under_a_wide_sky(hip_ctx_factory):
    """relMSE (mean (x - ref)^2 / (ref^2 + 0.01)) of the 64-spp films against the mean of the two modes'
    8,192-spp renders: MIS is below today's estimator.  Only the order is asserted; the values are logged."""
    W = H = 32
    depth, spp, ref_spp = 3, 64, 8192
    tiles = [(0, 0, W, H)]
    out = {}
    with hip_ctx_factory(0) as ctx:
        scene.upload_scene(ctx, scene.compile_scene(glossy_floor_scene((W, H))))
        for mis in (0, 1):
            ctx.set_option("mis", mis)
            rad, w = ctx.render(spp, depth, tiles, W, H)
            out[mis] = rad / w[..., None]
            rad, w = ctx.render(ref_spp, depth, tiles, W, H)
            out[mis, "ref"] = rad.astype(np.float64) / w[..., None]
    ref = 0.5 * (out[0, "ref"] + out[1, "ref"])
    today, with_mis = relmse(out[0], ref), relmse(out[1], ref)
    gap = relmse(out[0, "ref"], out[1, "ref"])
    line = (f"glossy floor (roughness 0.1) under procedural_sky(64), {W}x{H}, max_depth {depth}, {spp} spp: relMSE "
            f"today {today:.5f}, mis {with_mis:.5f}, ratio {with_mis / today:.3f}; relMSE between the two "
            f"{ref_spp}-spp references {gap:.6f}")
    print(line)   # recorded in profiles/mis_measure.log
    assert with_mis < today, line


# ----------------------------------------------------------------------------- CLI, adapter
SDL = """
let grey = DiffuseMaterial {{ color: [0.725, 0.71, 0.68] }}
let lamp = EmissiveMaterial {{ color: [17, 12, 4] }}
export scene = Scene {{
    camera: PerspectiveCamera {{ fov: 15, position: [0, 1, 9], resolution: [40, 24] }},
    integrator: Path {{ spp: 4, max_depth: 3, tile_size: 16 }},
    output: "{out}",
    shapes: [ AkariMesh {{ path: "{mesh}", materials: [$grey, $grey, $grey, $grey, $grey, $grey, $grey, $lamp] }} ]
}}
"""


def test_cli_mis_with_env(tmp_path):
    from akari_amd import film
    sky = np.zeros((8, 16, 3), np.float32)
    sky[:4] = [0.4, 0.6, 1.0]
    sky[4:] = [0.1, 0.1, 0.1]
    film.write_pfm(tmp_path / "sky.pfm", sky, np.ones(sky.shape[:2], np.float32))
    imgs = []
    for flags in ([], ["--mis"]):
        out = tmp_path / f"o{len(flags)}.pfm"
        (tmp_path / "s.akari").write_text(SDL.format(out=out, mesh=CORNELL_MESH))
        assert render.main([str(tmp_path / "s.akari"), "--env", str(tmp_path / "sky.pfm"), "--env-res", "16"] + flags) == 0
        imgs.append(envmap.read_pfm(out))
    assert imgs[1].shape == (24, 40, 3) and np.all(np.isfinite(imgs[1])) and imgs[1].mean() > 0
    assert not np.array_equal(imgs[0], imgs[1]), "--mis changed nothing"


def test_cpp_adapter_set_mis(tmp_path):
    exe = tmp_path / "mis_demo"
    lib = capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "mis_demo.cpp"), "-o",
                    str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    r = subprocess.run([str(exe), "run"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "form_wavefront=1 differs=1 weights_equal=1 continued_equals_fresh=1 refused=1" in r.stdout

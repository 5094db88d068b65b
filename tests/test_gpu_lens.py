"""The thin-lens camera on the device against its restatement.

tests/golden/lens_restate.py states the lens branch of kernel/camera.h:67-86 and the AO pixel loop in numpy f32;
tests/golden/make_lens_golden.py ran it into lens_golden_<scene>.npz.  The device has to give the same bits in
film, weight, final sampler state and (counting build) closest-hit and shadow ray counts, whatever options,
builder, session split or context split is used; a render with an active lens runs the wavefront form whatever
`path` says, an inactive lens changes nothing at all, and the cost-order pilot changes no bit of the film.
Every test here calls akr_hip_set_lens (upload_scene does), which the library did not have before.
"""
import subprocess
import sys

import numpy as np
import pytest

import py_oracle
from akari_amd import capi, envmap, progressive, render, scene
from conftest import CORNELL_MESH, GOLDEN, ROOT
from test_gpu_path_kat import probe_frame
from test_path_kat_host import M, check, compare_with_golden, golden

sys.path.insert(0, str(GOLDEN))
import lens_restate as L  # noqa: E402
import make_lens_golden as ML  # noqa: E402
import ref_restate as R  # noqa: E402
import lens_scenes  # noqa: E402

pytestmark = pytest.mark.gpu

PATH_SCENES = [n for n, c in ML.CONFIGS.items() if c[1] != "ao"]
PATH_FORCED = {"path": 1, "path_defer": 0, "path_spec": 0, "env_path": 1, "env_forms": 1, "path_auto_complex": 1}
K_PATH = {"path": 1, "path_defer": 0, "path_spec": 0}


def lens_golden(name):
    return np.load(GOLDEN / f"lens_golden_{name}.npz")


def upload(ctx, name, **build_kw):
    cs = scene.compile_scene(ML.build_scene(name))
    scene.upload_scene(ctx, cs, **build_kw)
    return cs


def render_and_compare(factory, name, what, counting=(0,), exact_cull=False, options=None, **build_kw):
    """Every configuration of the scene; `counting`: the values of count_tests to render with."""
    g = lens_golden(name)
    with factory(0) as ctx:
        for k, v in (options or {}).items():
            ctx.set_option(k, v)
        ctx.set_option("pixel_probe", 1)
        upload(ctx, name, **build_kw)
        assert ctx.lens()[2], "the scene's lens did not reach the context"
        for key, depth, clamp, mis in ML.CONFIGS[name][2]:
            H, W = g[key + "_weight"].shape
            mask = np.zeros((H, W), bool)
            ctx.set_option("mis", int(mis))
            for c in counting:
                ctx.set_option("count_tests", c)
                rad, w = ctx.render(ML.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp, exact_cull=exact_cull)
                rays = compare_with_golden(g, key, mask, rad, w, probe_frame(ctx, W, H), f"{name} {key} {what} count {c}")
                assert ctx.render_form()["form"] == "wavefront", ctx.render_form()
                if c:
                    assert rays, f"{what}: the counting build recorded no ray counts"


@pytest.mark.parametrize("name", PATH_SCENES)
def test_scenes_equal_golden_default_options(hip_ctx_factory, name):
    render_and_compare(hip_ctx_factory, name, "default options", counting=(0, 1))


@pytest.mark.parametrize("name", PATH_SCENES)
def test_scenes_equal_golden_path_forced_and_exact_cull(hip_ctx_factory, name):
    """`path` 1 (and every option that widens the persistent forms' reach) asks for the persistent kernel; an
    active lens runs the wavefront form and says so."""
    render_and_compare(hip_ctx_factory, name, "path 1 forced", options=PATH_FORCED)
    render_and_compare(hip_ctx_factory, name, "exact_cull", exact_cull=True)


@pytest.mark.parametrize("builder", ["sbvh", "lbvh"])
@pytest.mark.parametrize("name", PATH_SCENES)
def test_builders_equal_golden(hip_ctx_factory, name, builder):
    kw = {"sbvh": dict(builder=capi.BUILDER_SBVH), "lbvh": dict(builder=capi.BUILDER_LBVH)}[builder]
    render_and_compare(hip_ctx_factory, name, builder, **kw)


def test_cost_order_pilot_changes_no_bit(hip_ctx_factory):
    """The pilot keeps pinhole rays: it orders the camera-ray queue and nothing else.  Ordered and unordered give
    the golden's bits, and the ordered render says it was ordered."""
    name, (key, depth, clamp, _) = "lens_box", ML.CONFIGS["lens_box"][2][1]
    g = lens_golden(name)
    H, W = g[key + "_weight"].shape
    with hip_ctx_factory(0) as ctx:
        ctx.set_option("pixel_probe", 1)
        ctx.set_option("path_order_min_spp", 0)
        upload(ctx, name)
        for order, ordered in ((2, True), (0, False)):
            ctx.set_option("path_order", order)
            rad, w = ctx.render(ML.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
            assert ctx.render_form() == {"form": "wavefront", "ordered": ordered}, (order, ctx.render_form())
            compare_with_golden(g, key, np.zeros((H, W), bool), rad, w, probe_frame(ctx, W, H), f"path_order {order}")


# ----------------------------------------------------------------------------- sessions
def test_continue_and_film_variance_change_no_bit(hip_ctx_factory):
    name, (key, depth, clamp, _) = "lens_box", ML.CONFIGS["lens_box"][2][2]
    g = lens_golden(name)
    H, W = g[key + "_weight"].shape
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        ctx.set_option("pixel_probe", 1)
        ctx.render(2, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
        rad, w = ctx.render_continue(2, W, H)
        assert ctx.render_form()["form"] == "wavefront"
        check(rad, g[key + "_radiance"], "2 + 2 spp by render_continue: radiance")
        check(w, g[key + "_weight"], "2 + 2 spp by render_continue: weight")
        assert np.array_equal(probe_frame(ctx, W, H)["seed"], g[key + "_seed"]), "2 + 2 spp: final sampler states"
        ctx.set_option("film_variance", 1)
        rad, w = ctx.render(ML.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
        compare_with_golden(g, key, np.zeros((H, W), bool), rad, w, probe_frame(ctx, W, H), "film_variance on")
        assert ctx.render_variance(W, H).shape == (H, W, 4)


@pytest.mark.parametrize("name,key", [("lens_wide", "d5"), ("lens_sky_spec", "d4_mis")])
def test_two_context_split_equals_single(hip_ctx_factory, name, key):
    _, depth, clamp, mis = next(c for c in ML.CONFIGS[name][2] if c[0] == key)
    g = lens_golden(name)
    H, W = g[key + "_weight"].shape
    tiles = [(x, y, x + 8, y + 8) for y in range(0, H, 8) for x in range(0, W, 8)]
    with hip_ctx_factory(0) as a, hip_ctx_factory(0) as b:
        upload(a, name)
        upload(b, name)
        rad, w = capi.render_node([a, b], ML.SPP, depth, tiles, W, H, ray_clamp=clamp, mis=mis)
        check(rad, g[key + "_radiance"], "two-context render_node radiance")
        check(w, g[key + "_weight"], "two-context render_node weight")


_PREFIX = {}


def box_prefixes(cap, depth=5):
    """The restatement's lens_box film sums and sampler states after 0 .. cap samples of every pixel, run once: a
    slot's samples are one chain, so a slot that holds c samples equals entry c."""
    if cap not in _PREFIX:
        sc, _ = ML.restate_scene("lens_box")
        W, H = sc.camera.res
        film = np.zeros((cap + 1, H, W, 3), np.float32)
        seed = np.zeros((cap + 1, H, W), np.uint32)
        for y in range(H):
            for x in range(W):
                sampler, tr, rad = R.LCG(x + y * W), R.Tracer(sc), (R.F(0.0),) * 3
                seed[0, y, x] = sampler.seed
                for c in range(1, cap + 1):
                    rad = R.add(rad, R.path_sample(sc, sampler, x, y, depth, None, tr))
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
    film, seed, depth = box_prefixes(cap)
    H, W = seed.shape[1:]
    tiles = [(0, 0, W, H)]
    with hip_ctx_factory(0) as ctx:
        upload(ctx, "lens_box")
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


# ----------------------------------------------------------------------------- lens state
def cornell_k_path(ctx, what):
    """The unmodified Cornell golden, in the k_path form."""
    gp = golden("cornell")
    H, W = gp["mask"].shape
    rad, w = ctx.render(M.SPP, 5, [(0, 0, W, H)], W, H)
    assert ctx.render_form()["form"] == "k_path", (what, ctx.render_form())
    compare_with_golden(gp, "d5", gp["mask"], rad, w, probe_frame(ctx, W, H), what)


def test_inactive_lens_is_the_pinhole_in_the_k_path_form(hip_ctx_factory):
    g = lens_golden("lens_box")
    with hip_ctx_factory(0) as ctx:
        ctx.set_option("pixel_probe", 1)
        for k, v in K_PATH.items():
            ctx.set_option(k, v)
        scene.upload_scene(ctx, scene.compile_scene(M.build_scene("cornell")))
        assert ctx.lens() == (0.0, 0.0, False)            # a new context's, and what upload_scene sends for a pinhole
        cornell_k_path(ctx, "no lens")
        ctx.set_lens(0.3, 0.0)
        assert ctx.lens() == (float(np.float32(0.3)), 0.0, False)
        cornell_k_path(ctx, "set_lens(0.3, 0)")
        ctx.set_lens(0.0, 8.0)
        assert ctx.lens() == (0.0, 8.0, False)
        cornell_k_path(ctx, "set_lens(0, 8)")
        # a lens render on the same context (lens_box's camera and lens), then the pinhole again
        desc = ML.build_scene("lens_box")
        cam = desc.camera
        ctx.set_camera(cam.position, cam.rotation, cam.fov, cam.resolution)
        ctx.set_lens(cam.lens_radius, cam.focal_distance)
        H, W = g["d5_weight"].shape
        rad, w = ctx.render(ML.SPP, 5, [(0, 0, W, H)], W, H)
        assert ctx.render_form()["form"] == "wavefront"
        compare_with_golden(g, "d5", np.zeros((H, W), bool), rad, w, probe_frame(ctx, W, H), "lens_box by set_lens")
        pin = M.build_scene("cornell").camera
        ctx.set_camera(pin.position, pin.rotation, pin.fov, pin.resolution)
        assert ctx.lens()[2], "set_camera dropped the lens"
        ctx.set_lens(0.0, 0.0)
        cornell_k_path(ctx, "set_lens(0, 0) after a lens render")


def test_set_camera_keeps_the_lens_and_set_lens_ends_the_session(hip_ctx_factory):
    g = lens_golden("lens_box")
    H, W = g["d5_weight"].shape
    desc = ML.build_scene("lens_box")
    cam = desc.camera
    with hip_ctx_factory(0) as ctx:
        ctx.set_option("pixel_probe", 1)
        scene.upload_scene(ctx, scene.compile_scene(lens_scenes.pinhole(ML.build_scene("lens_box"))))
        assert not ctx.lens()[2]
        ctx.set_lens(cam.lens_radius, cam.focal_distance)
        ctx.set_camera(cam.position, cam.rotation, cam.fov, cam.resolution)      # after set_lens: the lens stays
        assert ctx.lens() == (float(np.float32(cam.lens_radius)), cam.focal_distance, True)
        rad, w = ctx.render(ML.SPP, 5, [(0, 0, W, H)], W, H)
        compare_with_golden(g, "d5", np.zeros((H, W), bool), rad, w, probe_frame(ctx, W, H), "set_camera after set_lens")
        ctx.set_lens(cam.lens_radius, cam.focal_distance)                         # even the same values end the session
        with pytest.raises(capi.AkrError, match="session"):
            ctx.render_continue(1, W, H)


@pytest.mark.parametrize("radius,focal,word", [(-0.1, 8.0, "lens_radius"), (float("nan"), 8.0, "lens_radius"),
                                               (float("inf"), 8.0, "lens_radius"), (0.3, -1.0, "focal_distance"),
                                               (0.3, float("nan"), "focal_distance"), (0.3, float("inf"), "focal_distance")])
def test_refused_set_lens_leaves_the_lens_and_the_session(hip_ctx_factory, radius, focal, word):
    g = lens_golden("lens_box")
    H, W = g["d5_weight"].shape
    with hip_ctx_factory(0) as ctx:
        ctx.set_option("pixel_probe", 1)
        upload(ctx, "lens_box")
        before = ctx.lens()
        ctx.render(2, 5, [(0, 0, W, H)], W, H)
        with pytest.raises(capi.AkrError, match=word):
            ctx.set_lens(radius, focal)
        assert ctx.lens() == before and before[2]
        rad, w = ctx.render_continue(2, W, H)                                    # the session stands, the lens too
        check(rad, g["d5_radiance"], "2 + 2 spp around a refused set_lens: radiance")
        check(w, g["d5_weight"], "2 + 2 spp around a refused set_lens: weight")
        assert np.array_equal(probe_frame(ctx, W, H)["seed"], g["d5_seed"])   # the probe's ray counts are the continue's alone


def test_lens_reads_back_what_was_set(hip_ctx_factory):
    with hip_ctx_factory(0) as ctx:
        assert ctx.lens() == (0.0, 0.0, False)
        for r, f in ((1e-30, 8.0), (1e3, 1e-3), (0.3, 1e6), (0.0, 0.0), (0.0, 2.0), (2.0, 0.0)):
            ctx.set_lens(r, f)
            assert ctx.lens() == (float(np.float32(r)), float(np.float32(f)), r > 0 and f > 0)


# ----------------------------------------------------------------------------- features, AO
def lens_camera_ray(cam, capi_, x, y, seed):
    """py_oracle.camera_ray's shape over the restated LensCamera: four draws of the chain, the ray, the new state."""
    s = R.LCG(seed)
    u1, u2 = s.next2d(), s.next2d()
    o, d = L.lens_camera_of(cam).generate_ray(u1, u2, (x, y))
    ray = np.zeros(1, capi_.RAY_DTYPE)
    ray["o"], ray["d"], ray["tmin"], ray["tmax"] = o, d, R.EPS, R.INF
    return ray[0], s.seed


def test_feature_pass_under_a_lens_and_the_filter_on_it(hip_ctx_factory, monkeypatch):
    """test_denoise_host.feature_reference with its camera rays from the restated LensCamera, traced by the oracle:
    the feature sums are blurred as the film is.  The filter runs on the result."""
    from test_denoise_host import feature_reference, frame_features
    desc = ML.build_scene("lens_box")
    cs = scene.compile_scene(desc)
    W, H = cs.camera.resolution
    tiles = [(0, 0, W, H)]
    with hip_ctx_factory(0) as ctx:
        scene.upload_scene(ctx, cs)
        nodes, tris = ctx.accel_export()
        orc = py_oracle.OracleScene(cs, nodes, tris, capi)
        pin = frame_features(feature_reference(cs, orc, tiles, 2), tiles, W, H)
        monkeypatch.setattr(py_oracle, "camera_ray", lens_camera_ray)
        want = frame_features(feature_reference(cs, orc, tiles, 2), tiles, W, H)
        got = ctx.render_features(2, tiles, W, H)
        assert np.array_equal(got, want), f"{np.count_nonzero(np.any(got != want, axis=-1))} pixels differ"
        assert np.count_nonzero(np.any(want != pin, axis=-1)) > W * H // 2, "the lens changed too few feature records"
        rad, w = ctx.render(ML.SPP, 5, tiles, W, H)
        out = ctx.denoise(rad, w, got)
        assert out.shape == (H, W, 3) and np.all(np.isfinite(out)) and out.mean() > 0


def test_ao_golden(hip_ctx_factory):
    g = lens_golden("lens_ao")
    H, W = g["ao_weight"].shape
    desc = ML.build_scene("lens_ao")
    with hip_ctx_factory(0) as ctx:
        scene.upload_scene(ctx, scene.compile_scene(desc))
        for exact_cull in (False, True):
            rad, w = ctx.render_ao(ML.SPP, [(0, 0, W, H)], W, H, occlude=desc.integrator.occlude, exact_cull=exact_cull)
            check(rad, g["ao_radiance"], f"AO radiance, exact_cull {exact_cull}")
            check(w, g["ao_weight"], "AO weight")
        ctx.set_lens(0.0, 0.0)
        rad, _ = ctx.render_ao(ML.SPP, [(0, 0, W, H)], W, H, occlude=desc.integrator.occlude)
        assert np.mean(np.any(rad != g["ao_radiance"], axis=-1)) >= 0.5       # what the generator measured as `differs`


# ----------------------------------------------------------------------------- CLI, adapter
SDL = """
let grey = DiffuseMaterial {{ color: [0.725, 0.71, 0.68] }}
let lamp = EmissiveMaterial {{ color: [17, 12, 4] }}
export scene = Scene {{
    camera: PerspectiveCamera {{ fov: 15, position: [0.3, 1.2, 9], rotation: [3, -2, 5], resolution: [24, 24]{lens} }},
    integrator: Path {{ spp: 4, max_depth: 5, tile_size: 8, ray_clamp: 0 }},
    output: "{out}",
    shapes: [ AkariMesh {{ path: "{mesh}", materials: [$grey, $grey, $grey, $grey, $grey, $grey, $grey, $lamp] }} ]
}}
"""


def run_cli(tmp_path, tag, lens_fields, *flags):
    out = tmp_path / f"{tag}.pfm"
    (tmp_path / "s.akari").write_text(SDL.format(out=out, mesh=CORNELL_MESH, lens=lens_fields))
    assert render.main([str(tmp_path / "s.akari"), *flags]) == 0
    return envmap.read_pfm(out)


def test_cli_lens_fields_flags_focus_and_gpus(tmp_path, capsys):
    pin = run_cli(tmp_path, "pin", "")
    by_field = run_cli(tmp_path, "field", ", lens_radius: 0.3, focal_distance: 8")
    by_flag = run_cli(tmp_path, "flag", "", "--lens-radius", "0.3", "--focal-distance", "8")
    assert np.array_equal(by_field, by_flag) and not np.array_equal(by_field, pin)
    assert by_field.shape == (24, 24, 3) and np.all(np.isfinite(by_field)) and by_field.mean() > 0
    capsys.readouterr()
    focused = run_cli(tmp_path, "focus", "", "--lens-radius", "0.3", "--focus-at", "12", "12")
    said = capsys.readouterr().out
    assert "focus at pixel (12, 12): focal distance" in said
    fd = float(said.split("focal distance")[1].split()[0])
    assert 7.0 < fd < 11.0 and np.all(np.isfinite(focused)) and not np.array_equal(focused, pin)
    again = run_cli(tmp_path, "again", "", "--lens-radius", "0.3", "--focal-distance", repr(fd))
    assert np.array_equal(focused, again), "--focus-at is --focal-distance with the printed value"
    denoised = run_cli(tmp_path, "dn", ", lens_radius: 0.3, focal_distance: 8", "--denoise")
    assert denoised.shape == by_field.shape and np.all(np.isfinite(denoised)) and not np.array_equal(denoised, by_field)
    if capi.device_count() >= 2:
        two = run_cli(tmp_path, "two", ", lens_radius: 0.3, focal_distance: 8", "--gpus", "2")
        assert np.array_equal(two, by_field), "--gpus 2 differs from one GPU"


def test_cli_focus_at_a_miss_names_the_pixel(tmp_path, capsys):
    (tmp_path / "s.akari").write_text(SDL.format(out=tmp_path / "o.pfm", mesh=CORNELL_MESH, lens="").replace(
        "position: [0.3, 1.2, 9], rotation: [3, -2, 5]", "position: [0.3, 1.2, 9], rotation: [90, 0, 0]"))
    with pytest.raises(SystemExit):
        render.main([str(tmp_path / "s.akari"), "--lens-radius", "0.3", "--focus-at", "3", "4"])
    assert "pixel (3, 4) hits nothing" in capsys.readouterr().err
    assert not (tmp_path / "o.pfm").exists()


def test_cpp_adapter_lens_demo(tmp_path):
    exe = tmp_path / "lens_demo"
    lib = capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "lens_demo.cpp"), "-o",
                    str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    r = subprocess.run([str(exe), "run"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("pinhole_sharp=1 form_wavefront=1 in_focus_sharp=1 defocus_blurs=1 bad_radius_refused=1 lens_kept=1 lens_off=1"
            in r.stdout)
